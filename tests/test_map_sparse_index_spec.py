"""CPU checks of `map`'s sparse reference index (dp_index_build_sparse): the per-id count rule its index query uses in place of
GetSharedIDs' word ladders, held against the oracle's GetSharedIDs; the refusals that come before any device call (a reference
longer than 2^31 - 1 bases, an index layout outside 0 - 2)."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O


# ---- the count rule (query_sparse_kernel / q_sparse_ids, dp_overlap.hip) ------------------------------------------------------

def _prepared(members, min_count):
    """The dense query kernel's set-list preparation for sets given as sorted id arrays (gather order = list order): the word
    range [start, i_last] of the early return, and for the 16-ladder the gather order after every drop event (word, first eight)."""
    n = len(members)
    first = [int(m[0]) // 64 if len(m) else 1 for m in members]  # (an empty IntSet keeps start 1, end 0)
    last = [int(m[-1]) // 64 if len(m) else 0 for m in members]
    lens = [x + 1 for x in last]
    start, end = min(first), max(last)
    i_last = end
    dstar = n - min_count + 1
    if 1 <= dstar <= n:
        i_last = min(i_last, max(start, sorted(lens)[dstar - 1]) - 1)
    events = []
    if min_count >= 13:
        tmp_id, tmp_len, cn = list(range(n)), list(lens), n
        shortest = min(tmp_len)
        i, fresh = start, True
        while i <= i_last:
            if shortest <= i:
                nxt_short = end
                j = 0
                while j < cn:
                    if tmp_len[j] <= i:
                        cn -= 1
                        tmp_id[j], tmp_len[j] = tmp_id[cn], tmp_len[cn]
                        continue
                    nxt_short = min(nxt_short, tmp_len[j])
                    j += 1
                shortest = nxt_short
                fresh = True
            if fresh:
                events.append((i, list(tmp_id[:8])))
                fresh = False
            i = max(shortest, i + 1)
    return start, i_last, events


def _rule_ids(members, min_count):
    """Candidates by the count rule; also how many ids the p7 term decided."""
    start, i_last, events = _prepared(members, min_count)
    if start > i_last:
        return [], 0
    lo, hi = start * 64, (i_last + 1) * 64
    holders = {}
    for j, m in enumerate(members):
        for x in m:
            if lo <= x < hi:
                holders.setdefault(int(x), []).append(j)
    ev_words = [w for w, _ in events]
    out, p7_decided = [], 0
    for x in sorted(holders):
        h = holders[x]
        c = len(h)
        if min_count <= 4:
            ok = c >= max(min_count, 1)
        elif min_count <= 12:
            ok = c >= min(min_count, 8)
        else:
            t = max(0, int(np.searchsorted(ev_words, x // 64, side="right")) - 1)
            f8 = events[t][1]
            p06 = any(j in f8[:7] for j in h)
            p7 = f8[7] in h
            c2 = c - (1 if (p7 and not p06) else 0)
            exact = min_count <= 24 or c >= min_count
            ok = c2 >= min(min_count, 16) and exact
            if exact and c >= min(min_count, 16) and not ok:
                p7_decided += 1
        if ok:
            out.append(x)
    return out, p7_decided


def _random_query(rng, aim_p7):
    """5 - 130 sets over up to 3 000 ids, some confined to narrow id ranges (drops, early returns); minCount 1 - 40 and never above
    the set count (Matches asks for int(0.25 n + 0.5) of n sets).  aim_p7: a 16-ladder query with ids planted in exactly
    minCount sets that include gather position 7 but none of 0 - 6."""
    n = int(rng.integers(24 if aim_p7 else 5, 131))
    M = int(rng.integers(200, 3000))
    mc = int(rng.integers(13, min(16, n) + 1)) if aim_p7 else int(rng.integers(1, min(40, n) + 1))
    members = []
    for j in range(n):
        if rng.random() < 0.03:
            members.append(set())
            continue
        a, b = 0, M
        if rng.random() < 0.35:  # ragged: a narrow window of the id range
            a = int(rng.integers(0, M - 64))
            b = min(M, a + int(rng.integers(64, 700)))
        size = int(rng.integers(1, 40))
        members.append(set(int(x) for x in rng.integers(a, b, size=size)))
    # ids many sets share (the higher regimes need counts near minCount)
    for _ in range(int(rng.integers(5, 40))):
        x = int(rng.integers(0, M))
        for j in rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False):
            members[int(j)].add(x)
    if aim_p7:
        for _ in range(int(rng.integers(1, 6))):
            x = int(rng.integers(0, M))
            for m in members:
                m.discard(x)
            for j in [7] + [int(v) for v in rng.choice(np.arange(8, n), size=mc - 1, replace=False)]:
                members[j].add(x)
    return [np.array(sorted(m), dtype=np.int64) for m in members], mc


def test_count_rule_matches_oracle_shared_ids():
    """The rule of the sparse index query - c >= max(minCount, 1) (minCount <= 4), c >= min(minCount, 8) (5 - 12),
    c' >= min(minCount, 16) with the p7 correction (>= 13), and c >= minCount above 24 - over 3 000 seeded queries against the
    oracle's GetSharedIDs(fast = true), every regime, drops and early returns; at least 20 queries in which the p7 term decides an
    id and 100 with minCount > 24."""
    rng = np.random.default_rng(20261016)
    n_queries, p7_queries, exact_queries, regimes = 3200, 0, 0, [0, 0, 0]
    for q in range(n_queries):
        members, mc = _random_query(rng, aim_p7=(q % 8 == 7))
        sets = []
        for m in members:
            s = O.IntSet()
            for x in m:
                s.add(int(x))
            sets.append(s)
        want = [int(x) for x in O.shared_ids(sets, mc, True)]
        got, decided = _rule_ids(members, mc)
        assert got == want, (q, mc, len(members))
        p7_queries += decided > 0
        exact_queries += mc > 24
        regimes[0 if mc <= 12 else 1 if mc <= 24 else 2] += 1
    print("queries %d: 4/8-ladder %d, 16-ladder %d, exact %d; p7 decided in %d" % (n_queries, *regimes, p7_queries))
    assert p7_queries >= 20
    assert exact_queries >= 100


# ---- refusals before any device call ----------------------------------------------------------------------------------------------

def _host():
    from downpore_amd.overlap import load_host
    H = load_host()
    H.dph_map_run_ex.restype = C.c_void_p
    H.dph_map_run_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    H.dph_last_error.restype = C.c_char_p
    return H


def _small_reads():
    from downpore_amd.overlap import Reads
    bases, off = O.gen_reads(3, 20000, 4, 2000, 0.0, False)
    return Reads(bases, off, min_len=500)


def test_reference_longer_than_2_31_is_refused_with_its_length():
    from downpore_amd import DpError
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    n = (1 << 31) + 64
    bases = np.full(n, ord("A"), dtype=np.uint8)
    bases[1::7] = ord("C")
    ref = Reads(bases, np.array([0, n], dtype=np.int64), min_len=0, himem=False)
    del bases
    reads = _small_reads()
    with pytest.raises(DpError) as e:
        map_reads(ref, reads)
    msg = str(e.value)
    assert str(n) in msg, msg
    # refused by the length check itself, not by a device call that failed (no device here, or one that was never touched)
    assert "device" not in msg.lower() and "hip" not in msg.replace("dph_", "").lower(), msg


@pytest.mark.parametrize("index", [3, -1, 7, "compact", None, 1.5, True])
def test_bad_index_layout_is_refused_before_any_device_call(index):
    from downpore_amd import DpError
    from downpore_amd.mapping import map_reads
    with pytest.raises(DpError) as e:
        map_reads(None, None, index=index)  # (no read set, no library call: the value alone is refused)
    assert "index" in str(e.value)


@pytest.mark.parametrize("layout", [3, -1, 1 << 40])
def test_host_abi_refuses_a_bad_layout(layout):
    H = _host()
    reads = _small_reads()
    p = np.array([1, 11, 1000, 500, 10000, 40, layout], dtype=np.int64)
    h = H.dph_map_run_ex(reads.h, reads.h, p.ctypes.data, 7, 0)
    assert not h
    msg = H.dph_last_error(None).decode()
    assert "layout" in msg and str(layout) in msg, msg
    assert not H.dph_map_run_ex(reads.h, reads.h, p.ctypes.data, 8, 0)  # (6 or 7 parameters)
