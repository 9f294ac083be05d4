"""The two device calls behind a mapper's trimmed batch.  dp_reads_replace_tail_packed puts a raw batch behind a resident head unpaired;
dp_reads_respan_tail_rc replaces that tail by the (span, reverse complement) pairs of spans of itself - source and destination are the
same region of one block.  Both are held to the host packer (plus reverse strands computed from codes) and to what a fresh context
holds after dp_reads_upload_rc of head + host-cut slices; the head must stay byte for byte, and what it is for - its chunk scan, on the
owner and through a borrowing context - must not notice either call.  Integers and bytes: equal means equal."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_reads_tail import _all_reads, _counts, _pack_block, _reads, _same_scan
from tests.test_gpu_reads_tail import genome_case  # noqa: F401  (the 150 kb head with its seeds and chunk items)
from tests.test_map_trim_cpu import SRC_LENS, pack, reverse_strand, sources
from tests.test_overlap_trim_gpu import _span_list

pytestmark = pytest.mark.gpu

BIG = len(SRC_LENS) - 1  # the 70 001-base source
HEADS = [[], [1], [64, 65, 1000]]


def _block(seqs):
    """byte strings in the host layout of dp_reads_upload_packed_rc, packed by the host packer (any alphabet)"""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    poff = np.concatenate([[0], np.cumsum(((lens.astype(np.int64) + 3) // 4 + 15) & ~15)])
    blk = np.zeros(int(poff[-1]), dtype=np.uint8)
    for r, s in enumerate(seqs):
        p = pack(s)
        blk[poff[r]:poff[r] + len(p)] = p
    return blk, lens


@pytest.fixture(scope="module")
def case():
    """the sources as a packed block, the spans (tests/test_map_trim_gpu.py::kernel_case's) and both strands of every span, made once"""
    seqs = sources()
    spans = [tuple(int(v) for v in sp) for sp in _span_list(seqs[:BIG])]  # every start % 16 x every length, shuffled; one source used twice
    n = len(seqs[BIG])
    big = [(BIG, 4096 * a + 16 * (a + ln) + a, ln) for a in range(16) for ln in (1, 15, 16, 17, 63, 64, 65)]  # every alignment, in many workgroups
    big.append((BIG, 5, n - 5))  # ... and to the end
    big = [big[i] for i in np.random.default_rng(8).permutation(len(big))]
    spans += big
    spans.append((BIG, 3, 69_990))   # one read that spans many workgroups
    spans.append((BIG, n - 17, 17))  # ends on the last base of the last read of the buffer
    spans = np.array(spans, dtype=np.uint32)
    assert len(spans) > 500 and set((spans[:, 1] % 16).tolist()) == set(range(16))
    assert (np.diff(spans[:, 0].astype(np.int64)) < 0).any()
    cuts = [seqs[r][st:st + ln] for r, st, ln in spans.tolist()]
    fw = [pack(c) for c in cuts]
    rv = [reverse_strand(p, len(c)) for p, c in zip(fw, cuts)]
    blk, lens = _block(seqs)
    return dict(seqs=seqs, blk=blk, lens=lens, spans=spans, cuts=cuts, fw=fw, rv=rv)


def _offset(spans, keep):
    sp = np.array(spans, dtype=np.uint32).reshape(-1, 3).copy()
    sp[:, 0] += keep
    return sp


def _head_context(head):
    """a context that holds the head and nothing behind it"""
    import downpore_amd
    ctx = downpore_amd.Context(0)
    blk, lens = _pack_block(head)
    ctx.upload_reads_packed_rc(blk, lens, len(head), pinned=True)
    assert _counts(ctx) == (len(head), sum(len(h) for h in head))
    return ctx


def _table_bytes(ctx):
    """the library's own idea of every read's packed size (its length table)"""
    L = ctx.L
    L.dp_reads_packed.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    out = []
    for d in range(_counts(ctx)[0]):
        n = C.c_uint64(0)
        buf = np.zeros(1, dtype=np.uint8)
        L.dp_reads_packed(ctx.h, d, buf.ctypes.data, 0, C.byref(n))  # (cap 0: the size alone; a read of no bytes is copied as nothing)
        out.append(int(n.value))
    return out


def _fresh_rc(head, cuts):
    """what a fresh context holds after dp_reads_upload_rc of head + host-cut slices, the slices paired"""
    import downpore_amd
    other = downpore_amd.Context(0)
    parts = [bytes(h) for h in head] + [bytes(c) for c in cuts]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    other.upload_reads_rc(np.frombuffer(b"".join(parts), dtype=np.uint8), off, len(head))
    got = _all_reads(other), _counts(other)
    other.close()
    return got


@pytest.mark.parametrize("head_lens", HEADS, ids=["keep0", "keep1", "keep3"])
def test_raw_tail_then_spans_of_it_equal_the_host_and_a_fresh_upload(case, head_lens):
    keep = len(head_lens)
    head = _reads(np.random.default_rng(40 + keep), head_lens)
    seqs, spans = case["seqs"], case["spans"]
    ctx = _head_context(head)
    try:
        head_before = [bytes(ctx.packed_read(d)) for d in range(keep)]
        table_before = _table_bytes(ctx)
        assert table_before == [(n + 3) // 4 for n in head_lens]
        # ---- the raw batch, unpaired
        ctx.replace_tail_packed(keep, case["blk"], case["lens"])
        assert _counts(ctx) == (keep + len(seqs), sum(head_lens) + sum(SRC_LENS))
        for r, s in enumerate(seqs):
            assert np.array_equal(ctx.packed_read(keep + r), pack(s)), r
        assert [bytes(ctx.packed_read(d)) for d in range(keep)] == head_before
        assert _table_bytes(ctx) == table_before + [(n + 3) // 4 for n in SRC_LENS]
        # ---- spans of it, paired, in its place
        ctx.respan_tail_rc(keep, _offset(spans, keep))
        n_out = len(spans)
        assert _counts(ctx) == (keep + 2 * n_out, sum(head_lens) + 2 * int(spans[:, 2].sum()))
        got = _all_reads(ctx)
        for i in range(n_out):
            assert got[keep + 2 * i] == bytes(case["fw"][i]), (i, "host packer")
            assert got[keep + 2 * i + 1] == bytes(case["rv"][i]), (i, "reverse strand from codes")
        want, wc = _fresh_rc(head, case["cuts"])
        assert _counts(ctx) == wc and len(got) == len(want)
        bad = [d for d in range(len(want)) if got[d] != want[d]]
        assert not bad, bad[:8]
        assert got[:keep] == head_before
        assert _table_bytes(ctx)[:keep] == table_before
    finally:
        ctx.close()


def test_a_tail_that_outgrows_the_block_and_an_empty_one_leave_the_head_alone(case):
    head = _reads(np.random.default_rng(3), [64, 65, 1000])
    keep = len(head)
    ctx = _head_context(head)
    try:
        head_before = [bytes(ctx.packed_read(d)) for d in range(keep)]
        src = case["seqs"][10]  # 1000 bases: 256 bytes a strand
        blk, lens = _block([src])
        ctx.replace_tail_packed(keep, blk, lens)
        # 300 pairs of the whole read and of a slice at an odd alignment: some 150 KB behind a block that held less than 2 KB
        spans = [(keep, 0, 1000), (keep, 7, 993)] * 150
        ctx.respan_tail_rc(keep, np.array(spans, dtype=np.uint32))
        whole, part = pack(src), pack(src[7:])
        want = [bytes(whole), bytes(reverse_strand(whole, 1000)), bytes(part), bytes(reverse_strand(part, 993))] * 150
        assert _counts(ctx) == (keep + 600, sum(len(h) for h in head) + 300 * (1000 + 993))
        got = _all_reads(ctx)
        assert got[:keep] == head_before and got[keep:] == want
        # spans of the new tail, reverse strands among the sources
        ctx.respan_tail_rc(keep, np.array([(keep + 1, 0, 1000), (keep + 599, 1, 16)], dtype=np.uint32))
        rev = reverse_strand(part, 993)
        sl = np.unpackbits(rev)[2:34]  # its bases 1 .. 16
        got = _all_reads(ctx)
        assert got[:keep] == head_before and len(got) == keep + 4
        assert got[keep] == want[1] and got[keep + 1] == want[0]
        assert got[keep + 2] == bytes(np.packbits(sl))
        # n_out = 0
        ctx.respan_tail_rc(keep, np.zeros((0, 3), dtype=np.uint32))
        assert _counts(ctx) == (keep, sum(len(h) for h in head)) and _all_reads(ctx) == head_before
        ctx.replace_tail_packed(keep, blk, lens)  # ... and the next batch goes behind it as ever
        assert _all_reads(ctx) == head_before + [bytes(whole)]
    finally:
        ctx.close()


def test_ten_rounds_in_a_row():
    """raw tail, spans of it, the next raw tail - batches that grow and shrink - on one context"""
    rng = np.random.default_rng(12)
    head = _reads(rng, [20001, 2000])
    keep = 2
    ctx = _head_context(head)
    try:
        head_before = [bytes(ctx.packed_read(d)) for d in range(keep)]
        for i in range(10):
            n = 110 if i % 2 == 0 else 9
            batch = _reads(rng, rng.integers(1, 2500 if i % 2 == 0 else 90, n))
            blk, lens = _pack_block(batch)
            ctx.replace_tail_packed(keep, blk, lens)
            raw = _all_reads(ctx)
            blk1, _ = _pack_block(batch[-1:])
            assert raw[:keep] == head_before and len(raw) == keep + n and raw[-1] == bytes(blk1[:(len(batch[-1]) + 3) // 4]), i
            spans = []
            for _ in range(2 * n):  # any order, reads used more than once, reads left out
                r = int(rng.integers(0, n))
                st = int(rng.integers(0, len(batch[r])))
                spans.append((r, st, int(rng.integers(1, len(batch[r]) - st + 1))))
            ctx.respan_tail_rc(keep, _offset(spans, keep))
            want, wc = _fresh_rc(head, [batch[r][st:st + ln] for r, st, ln in spans])
            got = _all_reads(ctx)
            assert _counts(ctx) == wc and got == want, i
            assert got[:keep] == head_before
    finally:
        ctx.close()


def test_a_short_batch_after_a_long_one_reads_nothing_of_it(genome_case):  # noqa: F811
    """The 64 bytes behind the last read must be zero again when a short tail follows a long one.  They cannot be read through the ABI;
    what reads them is a scan of the last read, so both strands of it are scanned here and in a context that never held the long tail."""
    import downpore_amd
    g = genome_case
    k = g["k"]
    keep = 2
    long_batch, short = g["batches"][1], g["batches"][0][:3]
    L = len(short[-1])
    fresh = _head_context(g["head"])
    ctx = _head_context(g["head"])
    try:
        for c in (fresh, ctx):
            c.round_begin(k, g["seeds"])
        sblk, slens = _pack_block(short)
        # raw tail: the last read is device read keep + 2
        lblk, llens = _pack_block(long_batch)
        ctx.replace_tail_packed(keep, lblk, llens)
        ctx.replace_tail_packed(keep, sblk, slens)
        fresh.replace_tail_packed(keep, sblk, slens)
        win = np.array([(keep + 2, 0, L - k + 1, 0), (keep + 2, L - 200, 200 - k + 1, 0)], dtype=np.uint32)
        want = fresh.scan(win)
        assert want["n_seeds"].sum() > 10 and _same_scan(ctx.scan(win), want)
        # spans: a long paired tail, then a short one whose last pair is the whole last read
        ctx.replace_tail_packed(keep, lblk, llens)
        ctx.respan_tail_rc(keep, np.array([(keep + r, 0, len(b)) for r, b in enumerate(long_batch)], dtype=np.uint32))
        ctx.replace_tail_packed(keep, sblk, slens)
        sp = np.array([(keep + r, 0, len(b)) for r, b in enumerate(short)], dtype=np.uint32)
        ctx.respan_tail_rc(keep, sp)
        fresh.respan_tail_rc(keep, sp)
        last = keep + 2 * len(short) - 1  # the reverse strand of the last read: the last bytes of the block
        win = np.array([(last - 1, 0, L - k + 1, 0), (last, 0, L - k + 1, 0), (last, L - 200, 200 - k + 1, 0)], dtype=np.uint32)
        want = fresh.scan(win)
        assert want["n_seeds"].sum() > 10 and _same_scan(ctx.scan(win), want)
        assert _all_reads(ctx)[keep:] == _all_reads(fresh)[keep:]
    finally:
        ctx.close()
        fresh.close()


def test_refusals_name_the_call_and_the_reason_and_change_nothing(case):
    import downpore_amd
    from downpore_amd.hip import DpError
    head = _reads(np.random.default_rng(5), [64, 65])
    keep = 2
    ctx = _head_context(head)
    w = None
    try:
        blk, lens = _block(case["seqs"][:11])
        ctx.replace_tail_packed(keep, blk, lens)
        before, cb = _all_reads(ctx), _counts(ctx)
        assert cb[0] == 13
        one = np.array([(keep, 0, 1)], dtype=np.uint32)

        def unchanged(c=ctx):
            assert _counts(c) == cb and _all_reads(c) == before

        with pytest.raises(DpError, match="dp_reads_replace_tail_packed: keep 14 is beyond the 13 device reads"):
            ctx.replace_tail_packed(14, blk, lens)
        unchanged()
        with pytest.raises(DpError, match="dp_reads_replace_tail_packed: read length out of range"):
            ctx.replace_tail_packed(keep, blk[:16], np.array([0x80000000], dtype=np.uint32))
        unchanged()
        with pytest.raises(DpError, match="dp_reads_respan_tail_rc: keep 14 is beyond the 13 device reads"):
            ctx.respan_tail_rc(14, one)
        unchanged()
        with pytest.raises(DpError, match=r"dp_reads_respan_tail_rc: span 1 names read 1 of the head \(keep 2\)"):
            ctx.respan_tail_rc(keep, np.array([(keep, 0, 1), (1, 0, 1)], dtype=np.uint32))
        unchanged()
        with pytest.raises(DpError, match="dp_reads_respan_tail_rc: span 1 lies outside its read"):
            ctx.respan_tail_rc(keep, np.array([(keep, 0, 1), (keep + 10, 990, 11)], dtype=np.uint32))
        unchanged()
        with pytest.raises(DpError, match="dp_reads_respan_tail_rc: span 0 lies outside its read"):
            ctx.respan_tail_rc(keep, np.array([(13, 0, 1)], dtype=np.uint32))
        unchanged()
        # more than 2^31 - 1 device reads: refused on the counts alone, before a span or a length is looked at
        L = ctx.L
        L.dp_reads_respan_tail_rc.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.dp_reads_replace_tail_packed.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        with pytest.raises(DpError, match="dp_reads_respan_tail_rc: too many reads"):
            ctx._chk(L.dp_reads_respan_tail_rc(ctx.h, keep, one.ctypes.data, 0x40000000))
        unchanged()
        with pytest.raises(DpError, match="dp_reads_replace_tail_packed: too many reads"):
            ctx._chk(L.dp_reads_replace_tail_packed(ctx.h, keep, blk.ctypes.data, lens.ctypes.data, 0x7ffffffe))
        unchanged()
        # a context that borrows its reads
        w = downpore_amd.Context(0, shared_from=ctx)
        w.read_len = np.array(ctx.read_len)
        with pytest.raises(DpError, match="dp_reads_respan_tail_rc on a context that borrows its reads"):
            w.respan_tail_rc(keep, one)
        with pytest.raises(DpError, match="dp_reads_replace_tail_packed on a context that borrows its reads"):
            w.replace_tail_packed(keep, blk, lens)
        unchanged()
        unchanged(w)
        w.close()
        w = None
        # a read set of dp_reads_upload_rc_begin stays pending until the owner's final wait
        L.dp_reads_upload_rc_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.dp_reads_upload_wait.argtypes = [C.c_void_p, C.c_uint32]
        seqs = case["seqs"][:11]
        bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        travelling = downpore_amd.Context(0)
        try:
            travelling._chk(L.dp_reads_upload_rc_begin(travelling.h, bases.ctypes.data, off.ctypes.data, 11, 11, 11))
            travelling.read_len = np.diff(off)
            with pytest.raises(DpError, match="dp_reads_respan_tail_rc while an upload of dp_reads_upload_rc_begin is pending"):
                travelling.respan_tail_rc(0, np.array([(0, 0, 1)], dtype=np.uint32))
            travelling._chk(L.dp_reads_upload_wait(travelling.h, 0xffffffff))
            assert _counts(travelling) == (11, sum(SRC_LENS[:11])) and _all_reads(travelling) == before[keep:]
            travelling.respan_tail_rc(0, np.array([(0, 0, 1)], dtype=np.uint32))  # (the upload joined, the call goes through)
            assert _counts(travelling) == (2, 2)
        finally:
            travelling.close()
    finally:
        if w is not None:
            w.close()
        ctx.close()


def test_the_head_chunk_scan_survives_both_calls(genome_case):  # noqa: F811
    g = genome_case
    ctx = _head_context(g["head"])
    try:
        ctx.round_begin(g["k"], g["seeds"])
        before = ctx.scan(g["items"])
        assert before["n_seeds"].sum() > 1000
        rng = np.random.default_rng(6)
        for batch in (g["batches"][1], g["batches"][0][:5], g["batches"][1]):
            blk, lens = _pack_block(batch)
            ctx.replace_tail_packed(2, blk, lens)
            assert _same_scan(ctx.scan(g["items"]), before)
            spans = [(2 + r, 10, len(b) - 20) for r, b in enumerate(batch) if len(b) > 40]
            spans = [spans[i] for i in rng.permutation(len(spans))]
            ctx.respan_tail_rc(2, np.array(spans, dtype=np.uint32))
            assert _same_scan(ctx.scan(g["items"]), before)
        ctx.respan_tail_rc(2, np.zeros((0, 3), dtype=np.uint32))
        assert _same_scan(ctx.scan(g["items"]), before)
    finally:
        ctx.close()


def test_borrowers_are_stale_after_either_call_until_refreshed(genome_case):  # noqa: F811
    import downpore_amd
    from downpore_amd.hip import DpError
    g = genome_case
    k = g["k"]
    own = _head_context(g["head"])
    w = None
    try:
        own.round_begin(k, g["seeds"])
        chunks = own.scan(g["items"])
        w = downpore_amd.Context(0, shared_from=own)
        w.read_len = np.array(own.read_len)
        w.round_begin(k, g["seeds"])
        assert _same_scan(w.scan(g["items"]), chunks)
        batch = g["batches"][1]  # many times the head's slack: the packed block moves
        blk, lens = _pack_block(batch)

        def stale():
            for call in (lambda: w.scan(g["items"][:1]), lambda: w.packed_read(0)):
                with pytest.raises(DpError, match=r"error -3: .*dp_ctx_refresh_shared"):
                    call()

        own.replace_tail_packed(2, blk, lens)
        stale()
        w.refresh_shared(own)
        assert _counts(w) == _counts(own) == (2 + len(batch), _counts(own)[1])
        assert _same_scan(w.scan(g["items"]), chunks)
        assert bytes(w.packed_read(2 + 57)) == bytes(own.packed_read(2 + 57))
        spans = np.array([(2 + r, 5, len(b) - 5) for r, b in enumerate(batch)], dtype=np.uint32)
        own.respan_tail_rc(2, spans)
        stale()
        w.refresh_shared(own)
        assert _counts(w) == _counts(own) and _counts(own)[0] == 2 + 2 * len(batch)
        assert _same_scan(w.scan(g["items"]), chunks)
        L = len(batch[57]) - 5
        win = np.array([(2 + 2 * 57, 0, L - k + 1, 0), (2 + 2 * 57 + 1, 0, L - k + 1, 0)], dtype=np.uint32)
        got, want = w.scan(win), own.scan(win)
        assert want["n_seeds"].sum() > 10 and _same_scan(got, want)
        assert bytes(w.packed_read(2 + 2 * 57 + 1)) == bytes(own.packed_read(2 + 2 * 57 + 1))
        assert w.n_seeds == len(g["seeds"])
    finally:
        if w is not None:
            w.close()
        own.close()
