"""The resident k-mer position index (dp_kbuild.hip: kb_count1, kb_part1, kb_count2, kb_part2, kb_final, and the atomic
count / scatter build of dp_kindex.hip) bucket by bucket against the plain numpy reference of tests/kindex_cases.py, on that file's
crafted read sets (tests/test_kindex_cases_cpu.py proves, without a GPU, that each case is where its name says).

Per case: the settings of the case for the block, upload, dp_scan_prepare, dp_kindex_dump; the build path the device reports (radix or
atomic scatter) and its geometry are the restated width rule's - a silent fallback is a failure, not a pass -; n_pos, off, the
histogram and every bucket's entries are the reference's; dp_kindex_digest is the same digest computed in numpy from the reference.
Everything is integer-exact.

Not covered here: read sets large enough to raise b2 above 6 (more than 128 Mbases) - tests/test_gpu_full_size.py stays the only cover
there - and RCCL between real GPUs.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from tests import kindex_cases as KC

pytestmark = pytest.mark.gpu

INFO = ("n_pos", "pos_fmt", "pbits", "sorted", "b1", "b2", "r", "rbits", "have_counts")


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


def _lib():
    from downpore_amd import hip
    L = hip.load_library()
    L.dp_kindex_dump.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dp_kindex_digest.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dp_comm_init_local.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dp_kindex_set_comm.argtypes = [C.c_void_p, C.c_void_p]
    L.dp_comm_destroy.argtypes = [C.c_void_p]
    return L


@pytest.fixture()
def ctx():
    from downpore_amd import hip
    _lib()
    c = hip.Context(0)
    yield c
    c.close()


def dump(ctx, k, phase=-1, tables=True):
    """dp_kindex_dump -> (info dict, off, entries, counts or None); tables = False: the entries alone"""
    info = np.zeros(len(INFO), dtype=np.uint64)
    ctx._chk(ctx.L.dp_kindex_dump(ctx.h, k, phase, info.ctypes.data, None, None, None))  # (sizes first)
    d = dict(zip(INFO, (int(x) for x in info)))
    nk = 4 ** k
    off = np.empty(nk + 1, dtype=np.uint64) if tables else None
    counts = np.empty(nk, dtype=np.uint32) if tables and d["have_counts"] else None
    entries = np.full(d["n_pos"], 0xdeaddeaddeaddead, dtype=np.uint64)
    ctx._chk(ctx.L.dp_kindex_dump(ctx.h, k, phase, info.ctypes.data, off.ctypes.data if tables else None, entries.ctypes.data,
                                  counts.ctypes.data if counts is not None else None))
    assert dict(zip(INFO, (int(x) for x in info))) == d
    return d, off, entries, counts


def check_path(tag, info, g):
    """the build path and geometry the device reports against the restated rule: no silent fallback"""
    if g.sorted and not info["sorted"]:
        pytest.fail("%s: the radix build was expected and the atomic scatter ran - dp_kindex_build_sorted's guard on free device memory "
                    "(free_b) is the one reason the width rule does not know; the case proves nothing on this machine" % (tag,))
    assert bool(info["sorted"]) == g.sorted, (tag, info)
    want = dict(pos_fmt=g.fmt, pbits=g.pbits, b1=g.b1, b2=g.b2, r=g.r, rbits=g.rbits if g.sorted else 0)
    assert {key: info[key] for key in want} == want, (tag, info)
    assert info["have_counts"] == (1 if g.sorted else 0), (tag, info)  # (the atomic scatter uses its counts up as cursors)


def check_index(tag, ctx, k, ref, g, phases=(-1,)):
    """dump, path, comparison with the reference, digest -> the info block"""
    info, off, entries, counts = dump(ctx, k, phases[0])
    check_path(tag, info, g)
    msg = KC.compare(ref, info["n_pos"], off, entries, counts)
    assert msg is None, (tag, "phase %d" % phases[0], msg)
    for ph in phases[1:]:  # (the same memory through another reader: the same array, slot for slot)
        _, _, e2, _ = dump(ctx, k, ph, tables=False)
        if not np.array_equal(e2, entries):
            i = int(np.flatnonzero(e2 != entries)[0])
            pytest.fail("%s: phase %d reads entry %d as %#x, phase %d as %#x" % (tag, ph, i, int(e2[i]), phases[0], int(entries[i])))
    got = np.zeros(3, dtype=np.uint64)
    ctx._chk(ctx.L.dp_kindex_digest(ctx.h, k, got.ctypes.data))
    assert [int(x) for x in got] == KC.digest(k, ref, ref.entries, ref.kmer), (tag, "dp_kindex_digest")
    return info


def upload(ctx, name):
    reads = KC.read_set(name)
    ctx.upload_reads(*KC.to_upload(reads))
    return reads


ALL_PHASES = (-1, 0, 1, 2, 3)


@pytest.mark.parametrize("name", [c.name for c in KC.CASES])
def test_index_build_equals_the_reference(ctx, name):
    c = KC.CASE[name]
    env = KC.env_of(c)
    with _Env(env):
        reads = upload(ctx, c.reads)
        ctx.scan_prepare(c.k)
        g = KC.geometry(c.k, [len(r) for r in reads], env)
        assert g.sorted == c.want["sorted"]
        # every format-5 case through all four alignments of its byte stream; one case of the other two formats as well
        phases = ALL_PHASES if name in KC.FMT5 or name in ("reads_257", "pay41_fmt8", "atomic_by_setting") else (-1,)
        check_index(name, ctx, c.k, KC.reference_of(c.reads, c.k), g, phases)


def test_stale_buffers_of_an_earlier_build(ctx):
    """one context: k = 10 on set A, a smaller set B at k = 13, set A at k = 10 again - off / pos reused or replaced every time"""
    env = KC.env_of({})
    with _Env(env):
        for step, (name, k) in enumerate([("plain10", 10), ("stale_small", 13), ("plain10", 10)]):
            reads = upload(ctx, name)
            ctx.scan_prepare(k)
            check_index(("stale", step, name), ctx, k, KC.reference_of(name, k), KC.geometry(k, [len(r) for r in reads], env))


def test_stale_buffers_across_formats_and_paths(ctx):
    """the same on the formats' buffers: format 5 (a byte stream), then the atomic scatter into what is left, then format 4"""
    for step, (name, k, extra) in enumerate([("count_257", 10, {"DP_KB_MIN_PBITS": "31"}), ("stale_small", 10, {"DP_TUNE": "kindex_atomic=1"}),
                                             ("count_257", 10, {})]):
        env = KC.env_of(extra)
        with _Env(env):
            reads = upload(ctx, name)
            ctx.scan_prepare(k)
            check_index(("stale formats", step, name), ctx, k, KC.reference_of(name, k), KC.geometry(k, [len(r) for r in reads], env))


def test_histogram_hand_over_in_both_orders():
    """dp_kmer_values then the atomic build (which takes that call's counts), and the radix build then dp_kmer_values (which takes the
    build's): the same value table bit for bit, the same index"""
    from downpore_amd import hip
    _lib()
    name, k = "plain10", 10
    ref = KC.reference_of(name, k)
    lens = [len(r) for r in KC.read_set(name)]
    tables = []
    for order, extra in (("values first", {"DP_TUNE": "kindex_atomic=1"}), ("index first", {})):
        env = KC.env_of(extra)
        c = hip.Context(0)
        try:
            with _Env(env):
                upload(c, name)
                if order == "values first":
                    tables.append(c.kmer_values(k))
                    c.scan_prepare(k)
                else:
                    c.scan_prepare(k)
                    info = dump(c, k, tables=False)[0]
                    assert info["have_counts"] == 1
                    tables.append(c.kmer_values(k))
                info = check_index((order,), c, k, ref, KC.geometry(k, lens, env))
                assert info["sorted"] == (0 if order == "values first" else 1)
        finally:
            c.close()
    assert np.array_equal(tables[0].view(np.uint64), tables[1].view(np.uint64))


def test_reverse_strands(ctx):
    """dp_reads_upload_rc: the reference is made of the reads the device holds (dp_reads_packed), both strands"""
    k, first_paired = 10, 3
    fwd = KC.read_set("rc")
    env = KC.env_of({})
    with _Env(env):
        ctx.upload_reads_rc(*KC.to_upload(fwd), first_paired)
        lens = [int(x) for x in ctx.read_len]
        assert len(lens) == first_paired + 2 * (len(fwd) - first_paired)
        held = [KC.unpack(ctx.packed_read(r), lens[r]) for r in range(len(lens))]
        for i in (0, first_paired, len(fwd) - 1):  # (forward strands are the uploaded reads, the strand behind one its complement reversed)
            dev = i if i < first_paired else first_paired + 2 * (i - first_paired)
            assert np.array_equal(held[dev], fwd[i])
            if i >= first_paired:
                assert np.array_equal(held[dev + 1], 3 - fwd[i][::-1])
        ctx.scan_prepare(k)
        check_index(("rc",), ctx, k, KC.reference(held, k), KC.geometry(k, lens, env))


@pytest.mark.parametrize("name,world,empty", [("skew_share", 3, [1]), ("plain10", 2, [])])
def test_index_built_in_shares(name, world, empty):
    """in-process ranks: every rank's gathered index is the reference.  skew_share with three ranks leaves rank 1 without a digit:
    kidx_off_rebase over zero k-mers, empty ranges in the all-gathers"""
    import downpore_amd
    L = _lib()
    k = 10
    env = KC.env_of({})
    ref = KC.reference_of(name, k)
    reads = KC.read_set(name)
    g = KC.geometry(k, [len(r) for r in reads], env)
    sizes = KC.share_digits(ref, g.b1, world)[1]
    assert [q for q in range(world) if sizes[q] == 0] == empty
    with _Env(env):
        ctxs = [downpore_amd.Context(0) for _ in range(world)]
        for c in ctxs:
            upload(c, name)
        hs = (C.c_void_p * world)(*[c.h for c in ctxs])
        comms = (C.c_void_p * world)()
        assert L.dp_comm_init_local(hs, world, comms) == 0
        for r in range(world):
            assert L.dp_kindex_set_comm(ctxs[r].h, comms[r]) == 0
        errs = []

        def build(c):
            try:
                c.scan_prepare(k)  # collective
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=build, args=(c,)) for c in ctxs]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th), "a rank did not come back from the collective build"
        assert not errs, errs
        for r in range(world):
            check_index((name, "rank", r), ctxs[r], k, ref, g)
        for r in range(world):
            L.dp_kindex_set_comm(ctxs[r].h, None)
            L.dp_comm_destroy(comms[r])
            ctxs[r].close()
