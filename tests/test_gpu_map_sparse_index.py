"""`map` on the sparse reference index (dp_index_build_sparse): the same rows as the dense bit matrices, the oracle's PAF with
index="sparse" on every input of the dense path's parity tests, BASELINE config 3 at full size, the 375 Mb config-5 share in both
layouts, and a 2.1 Gb reference whose dense index (about 332 GB) could not be allocated on one GPU.  The whole file takes about
90 s on one MI355X (86.9 s measured, profiles/sparse_index.txt)."""
import hashlib
import os

import numpy as np
import pytest

from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


def first_diff(a, b):
    if a == b:
        return None
    la, lb = a.split("\n"), b.split("\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d:\n  got  %s\n  want %s" % (i, x, y)
    return "line counts differ: got %d want %d" % (len(la), len(lb))


# ---- 1. rows ------------------------------------------------------------------------------------------------------------------

def _chunk_scan(ctx, k, G, seed):
    """a reference of G bases as 10 kb chunks (1 kb overlap), seeds = the k-mers at every 37th base: the scan output both builds use"""
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    ctx.upload_reads(genome, np.array([0, G], dtype=np.int64))
    lut = np.zeros(256, dtype=np.uint64)
    for ch, v in {65: 0, 67: 1, 71: 2, 84: 3}.items():
        lut[ch] = v
    c = lut[genome]
    km = np.zeros(G - k + 1, dtype=np.uint64)
    for j in range(k):
        km = (km << np.uint64(2)) | c[j:G - k + 1 + j]
    seeds = np.unique(km[::37]).astype(np.uint32)
    ctx.round_begin(k, seeds)
    items = [(0, s, min(10000, G - s) - k + 1, 0) for s in range(0, G - 2000, 9000)]
    return ctx.scan(items), len(seeds)


def _all_rows(ctx, S, M):
    post, meta = [], ctx.index_meta()
    for s in range(S):
        words, cnt, st, en = ctx.posting_row(s)
        post.append(words)
        assert (cnt, st, en) == tuple(int(x) for x in meta[s][:3])
    sets = [ctx.seedset_row(i) for i in range(M)]
    return np.array(post), np.array(sets), meta


@pytest.mark.parametrize("k", [11, 13])
def test_sparse_rows_equal_dense_rows(k):
    """dp_index_build and dp_index_build_sparse over the same chunk scan: every posting row, every seed-set row and every
    {count, first word, last word, last + 1} row identical - for the whole index, and for a shard of it (chunks from 64 on, word base
    1) after dp_index_set_global.  The sparse index stays within 8 H + 32 (S + M) bytes (+ 64 MiB) and holds as many entries as
    the dense rows have bits; dp_find_overlaps refuses it."""
    from downpore_amd import Context, DpError
    ctx = Context(0)
    try:
        res, S = _chunk_scan(ctx, k, 1200000, 40 + k)
        so, ns = res["seg_off"][:-1], res["n_seeds"]
        M = len(ns)
        assert M > 128 and S > 20000
        ctx.index_build(so, ns)
        d_post, d_sets, d_meta = _all_rows(ctx, S, M)
        d_info = ctx.index_info()
        ctx.index_build_sparse(so, ns)
        s_post, s_sets, s_meta = _all_rows(ctx, S, M)
        s_info = ctx.index_info()
        assert np.array_equal(d_post, s_post) and np.array_equal(d_sets, s_sets) and np.array_equal(d_meta, s_meta)
        assert d_info["layout"] == "dense" and s_info["layout"] == "sparse"
        H = int(ns.sum())
        assert s_info["entries"] == int(d_meta[:, 0].sum()) > 0
        print("k=%d: S=%d M=%d H=%d entries=%d sparse %d B, dense %d B" % (k, S, M, H, s_info["entries"], s_info["device_bytes"],
                                                                           d_info["device_bytes"]))
        assert s_info["device_bytes"] <= 8 * H + 32 * (S + M) + (64 << 20)
        with pytest.raises(DpError, match="sparse"):
            ctx.find_overlaps(np.array([0, 1, 0], dtype=np.int32), np.array([0, 3], dtype=np.uint64), 0.25, k, 500)
        # a shard: chunks [64, M) with word base 1, the sets' global windows from the whole index
        lo = 64
        ctx.index_build(so[lo:], ns[lo:])
        ctx.index_set_global(d_meta, 1, M)
        d_post2, d_sets2, d_meta2 = _all_rows(ctx, S, M - lo)
        ctx.index_build_sparse(so[lo:], ns[lo:])
        local = ctx.index_meta()
        ctx.index_set_global(d_meta, 1, M)
        s_post2, s_sets2, s_meta2 = _all_rows(ctx, S, M - lo)
        assert np.array_equal(d_post2, s_post2) and np.array_equal(d_sets2, s_sets2) and np.array_equal(d_meta2, s_meta2)
        assert np.array_equal(d_meta2, d_meta)
        assert int(local[:, 0].sum()) == sum(bin(int(w)).count("1") for w in d_post2.ravel())  # (the shard's own counts before)
    finally:
        ctx.close()


# ---- 2. the oracle's PAF with index="sparse" ------------------------------------------------------------------------------------

_REGIMES = {}  # run id -> queries per regime (4/8-ladder, 16-ladder, exact count, BIG tier)


def _run(run_id, seed, G, N, L, e, variable, circular, k=11, short_reads=False, env=None, min_len=500, **kw):
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    saved = {n: os.environ.get(n) for n in (env or {})}
    os.environ.update(env or {})
    try:
        genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
        goff = np.array([0, G], dtype=np.int64)
        bases, off = O.gen_reads(seed, G, N, L, e, variable)
        if short_reads:  # (the reads test_map_short_reads_and_len_mod4_quirks appends)
            extra_b, extra_o = O.gen_reads(seed, G, 40, 1400, e, True)
            cut = [1200, 1600, 1996, 2000, 900, 1333]
            b2, o2 = [], [0]
            for i in range(40):
                ln = min(int(extra_o[i + 1] - extra_o[i]), cut[i % len(cut)])
                b2.append(extra_b[extra_o[i]:extra_o[i] + ln])
                o2.append(o2[-1] + ln)
            bases = np.concatenate([bases] + b2)
            off = np.concatenate([off, off[-1] + np.array(o2[1:], dtype=np.int64)])
        want, werr = O.map_run(O.ReadSet(genome, goff, min_len=0, himem=False), O.ReadSet(bases, off, min_len=min_len, himem=False),
                               circular=circular, k=k, min_length=min_len, **kw)
        got, gerr, st = map_reads(Reads(genome, goff, min_len=0, himem=False), Reads(bases, off, min_len=min_len, himem=False),
                                  circular=circular, k=k, min_length=min_len, index="sparse", **kw)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    d = first_diff(got, want)
    assert d is None, (run_id, d)
    assert gerr == werr
    ix = st["index"]
    assert ix["layout"] == "sparse", ix
    _REGIMES[run_id] = [ix["q_ladder8"], ix["q_ladder16"], ix["q_exact"], ix["q_big"]]
    return want, st


PAF_INPUTS = {  # the inputs of test_gpu_map.py's PAF parity tests
    "bit_exact_1": dict(seed=3, G=200000, N=300, L=8000, e=0.0, variable=False, circular=True),
    "bit_exact_2": dict(seed=4, G=150000, N=300, L=6000, e=0.05, variable=True, circular=True),
    "bit_exact_3": dict(seed=5, G=300000, N=200, L=9000, e=0.10, variable=True, circular=False),
    "short_reads": dict(seed=6, G=120000, N=100, L=5000, e=0.02, variable=True, circular=True, short_reads=True),
    "errors_15": dict(seed=6, G=250000, N=250, L=7000, e=0.15, variable=True, circular=True),
    "one_lane": dict(seed=5, G=300000, N=200, L=9000, e=0.10, variable=True, circular=False, env={"DP_TUNE": "map_one_lane=1"}),
    "big_tier": dict(seed=23, G=300000, N=50, L=20000, e=0.02, variable=False, circular=True, query_size=8000, seed_rate=10),
    "ladder8": dict(seed=21, G=400000, N=400, L=3600, e=0.05, variable=True, circular=True, query_size=500, seed_rate=80),
    # windows of 150 - 250 usable seeds: minCount above 24, the exact count
    "exact_count": dict(seed=24, G=300000, N=200, L=10000, e=0.05, variable=True, circular=True, query_size=4000, seed_rate=20),
}
MAP_FLAGS = [dict(query_size=500), dict(query_size=2000), dict(seed_rate=20), dict(seed_rate=80), dict(chunk_size=5000),
             dict(chunk_size=20000), dict(min_length=2000), dict(query_size=500, seed_rate=20, chunk_size=5000, min_length=2000)]
for _k in (11, 13):
    for _i, _kw in enumerate(MAP_FLAGS):
        _kw = dict(_kw)
        PAF_INPUTS["flag_k%d_%d" % (_k, _i)] = dict(seed=21, G=400000, N=400, L=3600, e=0.05, variable=True, circular=True, k=_k,
                                                   min_len=_kw.pop("min_length", 500), **_kw)
for _shards, _G, _k, _e in ((3, 6000000, 11, 0.10), (4, 2600000, 9, 0.05), (2, 1500000, 13, 0.0)):
    PAF_INPUTS["shards_%d" % _shards] = dict(seed=11 + _shards, G=_G, N=400, L=7000, e=_e, variable=True, circular=True, k=_k,
                                             env={"DP_MAP_SHARDS": str(_shards)})


@pytest.mark.parametrize("run_id", sorted(PAF_INPUTS))
def test_sparse_map_matches_oracle(run_id):
    want, st = _run(run_id, **PAF_INPUTS[run_id])
    assert want.count("\n") > 0
    ix = st["index"]
    shards = int(PAF_INPUTS[run_id].get("env", {}).get("DP_MAP_SHARDS", "1"))
    per = ((int(st["n_chunks"]) + shards - 1) // shards + 63) // 64 * 64  # (whole 64-chunk words per shard: host_map.cpp)
    shards = (int(st["n_chunks"]) + per - 1) // per
    assert ix["index_builds"] == shards
    assert ix["index_bytes"] <= shards * (64 << 20) + 8 * ix["hits"] + 32 * shards * (st["n_seeds"] + st["n_chunks"])


def test_sparse_map_threads_borrow_one_index():
    """Several mapper threads (DP_MAP_THREADS, map_min_reads_per_thread): one sparse index, built once; the other contexts borrow
    it (no per-thread index, no per-batch import of the chunk segments).  The oracle's PAF."""
    env = {"DP_MAP_THREADS": "4", "DP_TUNE": "map_min_reads_per_thread=300", "DP_MAP_INFLIGHT": "500"}
    want, st = _run("threads", 5, 300000, 2600, 9000, 0.10, True, False, env=env)
    assert st["index"]["index_builds"] == 1
    assert st["n_batches"] >= 4


def test_sparse_runs_cover_every_regime():
    """Summed over the sparse runs of this file: at least 100 queries in each regime of the index query (4/8-ladder, 16-ladder,
    exact count, more than 512 sets).  Inputs not run yet in this session (this test selected alone) are run here."""
    for run_id in sorted(PAF_INPUTS):
        if run_id not in _REGIMES:
            _run(run_id, **PAF_INPUTS[run_id])
    tot = np.array(list(_REGIMES.values())).sum(axis=0)
    print("queries per regime over %d sparse runs: 4/8-ladder %d, 16-ladder %d, exact %d, BIG %d" % (len(_REGIMES), *tot))
    assert all(int(x) >= 100 for x in tot), tot


# ---- 3. config 3, 4. the config-5 share, 5. 2.1 Gb -------------------------------------------------------------------------------

def test_config3_full_size_sparse_matches_oracle():
    """BASELINE config 3 (50 000 reads x 8 kb at 10 % error, 4.6 Mb circular reference, k = 11) on the sparse index: the
    oracle's PAF, SHA-256 for SHA-256."""
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    G, N, L, e, seed = 4600000, 50000, 8000, 0.1, 3
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    bases, off = O.gen_reads(seed, G, N, L, e, False)
    want, werr = O.map_run(O.ReadSet(genome, goff, min_len=0, himem=False), O.ReadSet(bases, off, min_len=500, himem=False),
                           circular=True, k=11)
    got, gerr, st = map_reads(Reads(genome, goff, min_len=0, himem=False), Reads(bases, off, min_len=500, himem=False),
                              circular=True, k=11, index="sparse")
    assert st["index"]["layout"] == "sparse"
    assert want.count("\n") > N // 2
    assert hashlib.sha256(got.encode()).hexdigest() == hashlib.sha256(want.encode()).hexdigest()
    assert gerr == werr


def test_config5_share_sparse_equals_dense():
    """The 375 Mb config-5 share (k = 13, 1 000 reads x 15 kb at 10 % error): the sparse index in one context prints what the
    dense one prints, and so does the sparse index in eight shards (DP_MAP_SHARDS=8); the sparse index stays within
    8 H + 32 (S + M) + 64 MiB.  (The auto layout keeps this run dense: its 26 GB fit the device.)"""
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    from tools.synth import gen_reads_truth
    G, N, L, e, seed = 375000000, 1000, 15000, 0.1, 5
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    bases, off, starts, strands = gen_reads_truth(seed, G, N, L, e, False)
    ref = Reads(genome, goff, min_len=0, himem=False)
    reads = Reads(bases, off, min_len=500, himem=False)
    dense, derr, dst = map_reads(ref, reads, circular=True, k=13, index="auto")
    assert dst["index"]["layout"] == "dense", dst["index"]
    sparse, serr, sst = map_reads(ref, reads, circular=True, k=13, index="sparse")
    ix = sst["index"]
    print("config-5 share: dense %.1f s set-up, sparse %.1f s set-up; index %s" % (dst["t_setup_s"], sst["t_setup_s"], ix))
    assert ix["layout"] == "sparse" and ix["index_builds"] == 1
    assert ix["index_bytes"] <= 8 * ix["hits"] + 32 * (sst["n_seeds"] + sst["n_chunks"]) + (64 << 20)
    assert first_diff(sparse, dense) is None and serr == derr
    os.environ["DP_MAP_SHARDS"] = "8"
    try:
        sharded, sherr, shst = map_reads(ref, reads, circular=True, k=13, index="sparse")
    finally:
        del os.environ["DP_MAP_SHARDS"]
    assert shst["index"]["index_builds"] == 8
    assert first_diff(sharded, dense) is None and sherr == derr


def test_2100mb_reference_auto_layout_is_sparse():
    """A 2.1 Gb reference (k = 13, seed_rate 40, 10 kb chunks): its dense index - about 332 GB - exceeds the device, so the
    auto layout takes the sparse one.  The reported dense estimate exceeds the device's total memory, the sparse index stays
    within 8 H + 32 (S + M) + 64 MiB, and 2 000 reads x 15 kb at 10 % error map back to where the generator took them from
    (recall and precision >= 0.99)."""
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    from tools.synth import gen_reads_truth
    from tools.truth import map_truth
    G, N, L, e, seed = 2100000000, 2000, 15000, 0.1, 5
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    bases, off, starts, strands = gen_reads_truth(seed, G, N, L, e, False)
    got, gerr, st = map_reads(Reads(genome, goff, min_len=0, himem=False), Reads(bases, off, min_len=500, himem=False),
                              circular=True, k=13, index="auto")
    ix = st["index"]
    t = map_truth(got, off, starts, strands, G)
    print("2.1 Gb: set-up %.1f s, loop %.1f s (%.0f reads/s), index %s, truth %s" % (
        st["t_setup_s"], st["t_scan_s"] + st["t_chain_s"] + st["t_host_s"],
        N / max(1e-9, st["t_scan_s"] + st["t_chain_s"] + st["t_host_s"]), ix, t))
    assert ix["layout"] == "sparse"
    assert ix["dense_estimate"] > ix["device_total"] > 0
    assert ix["index_bytes"] <= 8 * ix["hits"] + 32 * (st["n_seeds"] + st["n_chunks"]) + (64 << 20)
    assert t["recall"] >= 0.99 and t["precision"] >= 0.99, t
