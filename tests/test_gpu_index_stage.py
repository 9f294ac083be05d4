"""A round's index build (dp_overlap.hip: chunk_kernel, index_fill_kernel, index_fill_rows_kernel + posting_transpose_kernel,
posting_meta_kernel, and their launch behind an un-waited scan) chunk by chunk, seed by seed against the oracle, on the crafted reads
of tests/index_cases.py (tests/test_index_cases_cpu.py proves, without a GPU, that each case is where its name says and that none of
them hands the device a walk without a bound).

Per case: the scan's survivors and segments are the plain scanner's; the chunks dp_index_build_chunked made are the oracle's pieces in
order - view, seeds, read, length, offset, inset - and fit the returned bound; dp_index_meta's four words of every seed, the posting
rows and the seed-set rows are those of the matrices built from the oracle's pieces, under both ways of filling them.  Everything is
integer-exact.
"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from tests import index_cases as IC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

FILL = [("atomics", "0"), ("rows", "1")]
REF_T = np.dtype([("seg_off", np.uint64), ("n_seeds", np.uint32), ("reserved", np.uint32)])
META_T = np.dtype([("read", np.uint32), ("length", np.int32), ("offset", np.int32), ("inset", np.int32)])


@pytest.fixture()
def ctx():
    from downpore_amd import hip
    c = hip.Context(0)
    L = c.L
    L.dp_index_build_chunked.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.dp_index_chunks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.dp_index_prechain.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_int32]
    L.dp_index_prechained.argtypes = [C.c_void_p]
    yield c
    c.close()


class _Env:
    """environment names set (or, value None, unset) for a block"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _err_code(name):
    hdr = open(os.path.join(O.ROOT, "include", "downpore_hip.h")).read()
    return int(re.search(name + r"\s*=\s*(-?\d+)", hdr).group(1))


def load(ctx, c):
    ctx.upload_reads(c.bases, c.off)
    ctx.round_begin(c.k, c.seed_kmers)


def scan(ctx, c, e, extra=None):
    """dp_scan_reads of the reads [e.lo, e.hi): survivors and their segments must be the plain scanner's -> the scan's result"""
    sc = ctx.scan_reads(np.zeros(c.n_reads, dtype=np.uint8), 1, e.lo, e.hi, False, c.scan_min, extra)
    assert np.array_equal(sc["read"], e.read), (c.name, "survivors")
    assert np.array_equal(sc["n_seeds"], e.n_seeds), (c.name, "hit counts")
    so = sc["seg_off"].astype(np.int64)
    ln = 2 * e.n_seeds + 1
    got = sc["segs"][np.repeat(so - e.seg_off, ln) + np.arange(ln.sum())]
    assert np.array_equal(got, e.segs), (c.name, "segments")
    return sc


def build(ctx, c, e, params=None):
    """dp_index_build_chunked for every survivor of the last scan -> the returned bound"""
    cap = C.c_uint32(0)
    p = params or (c.chunk_size, c.overlap, c.min_seeds, c.inset)
    ctx._chk(ctx.L.dp_index_build_chunked(ctx.h, p[0], p[1], p[2], p[3], len(e.read), C.byref(cap)))
    ctx.n_seqs = cap.value
    return cap.value


def _sample(rng, n, must, full):
    if n <= max(full, 1024):
        return np.arange(n)
    return np.unique(np.concatenate([rng.choice(n, 1024, replace=False), [x for x in must if 0 <= x < n]]))


def check_index(ctx, c, e, sc, cap, what):
    """chunks, meta and rows of the index on the context against the oracle's"""
    S, n = c.n_seeds, e.n_chunks
    tag = (c.name, what)
    # ---- the chunks
    assert n <= e.cap <= cap, tag
    refs, metas = np.zeros(cap + 4, dtype=REF_T), np.zeros(cap + 4, dtype=META_T)
    got_n = C.c_uint32(0)
    ctx._chk(ctx.L.dp_index_chunks(ctx.h, refs.ctypes.data, metas.ctypes.data, len(refs), C.byref(got_n)))  # (DP_ERR_CAPACITY raises)
    assert got_n.value == n, tag + ("chunk count", got_n.value, n)
    surv = e.chunks[:, 0]
    so = sc["seg_off"].astype(np.int64)
    first2 = refs["seg_off"][:n].astype(np.int64) - so[surv]
    assert np.all(first2 % 2 == 0) and np.array_equal(first2 // 2, e.chunks[:, 1]), tag + ("first seed",)
    assert np.array_equal(refs["n_seeds"][:n], e.chunks[:, 2]), tag + ("seeds",)
    assert np.array_equal(metas["read"][:n], e.read[surv]), tag + ("read",)
    for col, key in ((3, "length"), (4, "offset"), (5, "inset")):
        assert np.array_equal(metas[key][:n], e.chunks[:, col]), tag + (key,)
    # ---- every seed's {count, first word, last word, last + 1}
    assert np.array_equal(ctx.index_meta(), e.meta), tag + ("meta",)
    # ---- rows, word for word (W comes from the bound: a posting row holds no bit at or beyond the exact count either)
    W, SW = max(1, (cap + 63) // 64), max(1, (S + 63) // 64)
    rng = np.random.default_rng(7)
    last_seeds = e.e_seed[e.e_chunk == n - 1].tolist() if n else []
    seeds = _sample(rng, S, [0, S - 1, 63, 64, 65] + last_seeds, 4096 if n <= 4096 else 0)
    chunks = _sample(rng, n, [0, n - 1, 63, 64, 65], 4096 if S <= 4096 else 0)
    for s in seeds:
        words, cnt, st, en = ctx.posting_row(int(s))
        assert len(words) == W and np.array_equal(words, e.posting_row(int(s), W)), tag + ("posting row", int(s))
        assert (cnt, st, en) == tuple(int(x) for x in e.meta[s, :3]), tag + ("posting row meta", int(s))
    for i in chunks:  # (rows at or beyond the exact count are unspecified where rows are stored whole: never read)
        words = ctx.seedset_row(int(i))
        assert len(words) == SW and np.array_equal(words, e.seedset_row(int(i), SW)), tag + ("seed-set row", int(i))
    return len(seeds), len(chunks)


def run_case(ctx, name, env, what):
    c, e = IC.case(name), IC.expected(name)
    with _Env(env):
        load(ctx, c)
        sc = scan(ctx, c, e)
        cap = build(ctx, c, e)
        assert cap == e.cap, (name, what, "the bound is chunk_cap_of's sum")
        return check_index(ctx, c, e, sc, cap, what)


@pytest.mark.parametrize("fill", FILL, ids=[f[0] for f in FILL])
@pytest.mark.parametrize("name", [n for n in IC.SMALL_NAMES if n != "chained"] + list(IC.MATRIX_NAMES) + [IC.BIG_NAMES[0]])
def test_case_chunks_meta_and_rows(ctx, name, fill):
    run_case(ctx, name, {"DP_INDEX_FILL_ROWS": fill[1]}, fill[0])


@pytest.mark.parametrize("fill", FILL, ids=[f[0] for f in FILL])
def test_largest_case(ctx, fill):
    """66 000 chunks x 32 768 seeds: more rows than one pass of the row fill's grid, more wave tasks than one pass of the transpose's,
    two matrices of 270 MB each.  The only large case: on an MI355X 0.06 s on the device and comparing (1 034 posting rows, 1 029
    seed-set rows, every seed's meta), after about a second on the CPU for the oracle's 66 000 answers, shared by both fills."""
    name = IC.BIG_NAMES[1]
    IC.expected(name)
    t0 = time.time()
    rows = run_case(ctx, name, {"DP_INDEX_FILL_ROWS": fill[1]}, fill[0])
    print("%s %s: %.2f s on the device and comparing, %d posting and %d seed-set rows compared" % ((name, fill[0], time.time() - t0) + rows))


@pytest.mark.parametrize("name", IC.DEFAULT_MODE_NAMES)
def test_default_fill_on_either_side_of_its_threshold(ctx, name):
    """DP_INDEX_FILL_ROWS unset: rows from 4 M seed-set words up (8 192 chunks x 512 words), atomics below"""
    run_case(ctx, name, {"DP_INDEX_FILL_ROWS": None}, "default")


@pytest.mark.parametrize("order", [("1", "1"), ("1", "0"), ("0", "1")], ids=["rows_rows", "rows_atomics", "atomics_rows"])
def test_stale_buffers_on_one_context(ctx, order):
    """a large index, then a small one in the same buffers: the rows path clears nothing and has to overwrite every word it owns"""
    for name, fill in zip(("matrix_%dx%d" % IC.STALE[0], "matrix_%dx%d" % IC.STALE[1]), order):
        run_case(ctx, name, {"DP_INDEX_FILL_ROWS": fill}, "stale " + "/".join(order))


@pytest.mark.parametrize("fill", FILL, ids=[f[0] for f in FILL])
def test_chained_launches(ctx, fill):
    """dp_index_prechain: the stage launched by dp_scan_reads itself, behind the index step nobody has waited for, with grid, bound and W
    guessed from the context's previous round - and launched again by dp_index_build_chunked where a guess did not hold.  Ranges of one
    read set on one context (IC.CHAINED_ROUNDS; the CPU test holds each to what its label says); in every round chunks, meta and rows
    are the oracle's."""
    c = IC.case("chained")
    extra_reads = np.arange(4300, 4310)
    extra = np.array([(r, 0, min(100, c.off[r + 1] - c.off[r]) - c.k + 1, 0) for r in extra_reads], dtype=np.uint32)
    with _Env({"DP_SCAN_INDEX": "1", "DP_INDEX_FILL_ROWS": fill[1]}):
        ctx.upload_reads(c.bases, c.off)
        ctx.scan_prepare(c.k)
        prev = None
        for label, lo, hi, announce, with_extra, chained, bound in IC.CHAINED_ROUNDS:
            e = IC.expected("chained", lo, hi)
            ctx.round_begin(c.k, c.seed_kmers)
            if announce:
                ctx._chk(ctx.L.dp_index_prechain(ctx.h, c.chunk_size, c.overlap, c.min_seeds, c.inset))
            sc = scan(ctx, c, e, extra if with_extra else None)
            assert sc["index_mode"] == 1, label
            launched = ctx.L.dp_index_prechained(ctx.h)
            print("%s %s: dp_index_prechained() = %d" % (label, fill[0], launched))
            if chained is not None:
                assert launched == chained, label
            if with_extra:
                assert len(sc["extra_n_seeds"]) == len(extra) != 0
                for j, r in enumerate(extra_reads):
                    want = IC.expected_segments(c.bases[c.off[r]:c.off[r + 1]].tobytes().decode(), c.k, c.seed_kmers, 0, int(extra[j][2]) + c.k - 1)
                    at = int(sc["extra_seg_off"][j])
                    assert np.array_equal(sc["segs"][at:at + len(want)], want) and sc["extra_n_seeds"][j] == len(want) // 2, (label, j)
            cap = build(ctx, c, e)
            # "guess": the chained launch is used as it is; "exact": the stage was not launched, or was launched again for the exact bound
            assert cap == (IC.chain_guess(prev) if bound == "guess" else e.cap), (label, cap, e.cap, prev)
            check_index(ctx, c, e, sc, cap, label + " " + fill[0])
            prev = e.cap


def test_parameters_without_a_bound_are_refused(ctx):
    """6 <= min_seeds <= 100 and overlap / 2 <= chunk_size, or DP_ERR_ARG before anything is launched or armed.  The read is a short one
    that goes in whole: were the refusal missing, the kernel would still not enter the walk."""
    from downpore_amd.hip import DpError
    name = "matrix_1x257"
    c, e = IC.case(name), IC.expected(name)
    assert c.off[-1] < 200
    load(ctx, c)
    sc = scan(ctx, c, e)
    cap = C.c_uint32(77)
    for chunk_size, overlap, min_seeds in ((10000, 1000, 5), (10000, 1000, 0), (10000, 1000, 101), (10000, 20002, 6)):
        assert not IC.walk_bounded(chunk_size, overlap, min_seeds)
        for call in ("dp_index_build_chunked", "dp_index_prechain"):
            if call == "dp_index_prechain":
                rc = ctx.L.dp_index_prechain(ctx.h, chunk_size, overlap, min_seeds, 0)
            else:
                rc = ctx.L.dp_index_build_chunked(ctx.h, chunk_size, overlap, min_seeds, 0, len(e.read), C.byref(cap))
            assert rc == _err_code("DP_ERR_ARG"), (call, chunk_size, overlap, min_seeds)
            msg = ctx.L.dp_last_error(ctx.h).decode()
            assert msg.startswith(call + ":") and "6 <= min_seeds <= 100 and overlap / 2 <= chunk_size" in msg, msg
            with pytest.raises(DpError):
                ctx._chk(rc)
        assert cap.value == 77
    # nothing was armed: the next scan launches nothing, and the context builds a good index
    sc = scan(ctx, c, e)
    assert ctx.L.dp_index_prechained(ctx.h) == 0
    for fill in FILL:
        with _Env({"DP_INDEX_FILL_ROWS": fill[1]}):
            check_index(ctx, c, e, sc, build(ctx, c, e), "after the refusals, " + fill[0])
    # the limits themselves are accepted
    for chunk_size, overlap, min_seeds in ((10000, 20001, 6), (10000, 1000, 100)):
        build(ctx, c, e, (chunk_size, overlap, min_seeds, 0))
