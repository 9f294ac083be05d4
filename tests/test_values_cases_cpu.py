"""The crafted count tables of tests/values_cases.py on the CPU: the read set of a table counts back to the table, and the numpy model
(tests/values_model.py), the oracle's kmerValues and the product's host function kmerValuesFromCounts give one value table, bit for bit.
tests/test_gpu_values_table.py holds the device to the same model."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import values_cases as VC
from tests import values_model as M


def _host_values(counts, k):
    from downpore_amd.overlap import load_host
    H = load_host()
    H.dph_values_from_counts.restype = None
    H.dph_values_from_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    c = np.ascontiguousarray(counts, dtype=np.uint64).copy()
    got = np.zeros(4 ** k, dtype=np.float64)
    H.dph_values_from_counts(c.ctypes.data, k, got.ctypes.data)
    return got, c


def test_case_list_is_complete():
    """every family the cut is held to, on the path its name says"""
    names = VC.NAMES
    assert len(names) == len(set(names))
    for k in (4, 7, 8, 10):
        assert VC.path_of(VC.case("edge-of-histogram-k%d-T2046" % k)) == "histogram"
        assert VC.path_of(VC.case("edge-of-histogram-k%d-T2048" % k)) == "sort"
    for k in (8, 10):
        assert sum(n.startswith("tie-at-") and n.endswith("-k%d" % k) for n in names) == 8
    for fam in ("every-tie-falls", "one-tie-falls"):
        assert {VC.path_of(VC.case(n)) for n in names if n.startswith(fam)} == {"histogram", "sort"}
    assert {k for n, k in VC.CASES if n.startswith("sort-path")} == {5, 8, 9, 11}
    assert sorted(k for n, k in VC.CASES if n.startswith("each-k")) == list(range(4, 12))
    assert [k for n, k in VC.CASES if k > 11] == [13]


def test_edge_tables_differ_only_in_the_tied_level():
    for k in (4, 7, 8, 10):
        a, b = VC.case("edge-of-histogram-k%d-T2046" % k), VC.case("edge-of-histogram-k%d-T2048" % k)
        ma, mb = M.merged_counts(a.counts, k), M.merged_counts(b.counts, k)
        assert np.array_equal(ma == 2046, mb == 2048)
        assert np.array_equal(ma[ma != 2046], mb[mb != 2048])
        assert {key: a.info[key] for key in ("above", "ties", "cut_ties", "X")} == {key: b.info[key] for key in ("above", "ties", "cut_ties", "X")}


@pytest.mark.parametrize("name", [n for n in VC.NAMES if n != VC.SLICES])
def test_model_oracle_and_host_agree(name):
    c = VC.case(name)
    bases, off = M.reads_of(c.counts, c.k)
    assert len(off) - 1 == c.info["total"]
    rs = O.ReadSet(bases, off, min_len=0)
    assert np.array_equal(rs.kmer_counts(c.k), c.counts), "the reads of k bases do not count back to the table"
    want = rs.kmer_values(c.k)
    assert VC.first_difference(c, want) is None, "model against oracle: " + VC.first_difference(c, want)
    got, merged = _host_values(c.counts, c.k)
    assert VC.first_difference(c, got) is None, "host function against model: " + VC.first_difference(c, got)
    assert np.array_equal(merged.astype(np.int64), M.merged_counts(c.counts, c.k))


@pytest.mark.parametrize("k,G,N,L", [(4, 20000, 100, 1500), (8, 30000, 200, 3000), (10, 200000, 500, 4000)])
def test_model_matches_oracle_on_generated_reads(k, G, N, L):
    bases, off = O.gen_reads(60 + k, G, N, L, 0.01, True)
    rs = O.ReadSet(bases, off, min_len=0)
    table, info = M.values(rs.kmer_counts(k), k)
    want = rs.kmer_values(k)
    assert np.array_equal(table.view(np.uint64), want.view(np.uint64)), info
    assert (table > 0).sum() > 0


def test_rc_ids_against_the_oracle():
    for k in (4, 5, 8, 11, 13):
        rc = M.rc_ids(k)
        for i in (0, 1, 4 ** k - 1, 4 ** k // 3, 12345 % 4 ** k):
            assert int(rc[i]) == O.lib().dpo_rc_kmer(i, k)
        assert np.array_equal(rc[rc], np.arange(4 ** k, dtype=np.uint32))


def test_value_of_code_is_the_scalar_formula():
    total = 154029
    for code in (0, 1, 2, 3, 4, 254, 65535, 100000):
        freq = float(code) / float(total)
        want = 0.0 if code < 3 else (1.0 - (0.000005 - freq) if freq <= 0.000005 else 1.0 - (freq - 0.000005))
        assert float(M.value_of_code(code, total)) == want
    # both branches: a count of 3 in 10^6 reads lies under the target frequency
    assert float(M.value_of_code(3, 1000000)) == 1.0 - (0.000005 - 3.0 / 1000000.0)
