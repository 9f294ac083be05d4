"""The value table's 1 % cut on the device (dp_values.hip), table by table: every crafted count table of tests/values_cases.py goes to the
device as reads of k bases, and dp_kmer_histogram must give the table back and dp_kmer_values the model's value table
(tests/values_model.py), all 4^k entries bit for bit.  The cases place the threshold T on either side of the histogram's last bin (the
histogram path below VH_BINS, the sort path from it), the lowest cut tie X on tile, row and wave boundaries, make every tie fall or one,
and run both paths in one context one after the other.  The code downloads (dp_values_download_codes8 / dp_values_download_codes), their
overflow flags and their clamps are held to the same tables."""
import numpy as np
import pytest

from tests import values_cases as VC
from tests import values_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import downpore_amd
    c = downpore_amd.Context(0)
    yield c
    c.close()


def _run(ctx, c):
    """the case on the device: its reads, the histogram back, the value table against the model"""
    bases, off = M.reads_of(c.counts, c.k)
    ctx.upload_reads(bases, off)
    hist = ctx.kmer_histogram(c.k)
    assert np.array_equal(hist, c.counts), "%s: the device histogram is not the count table (first id %d)" % (
        c.name, int(np.flatnonzero(hist != c.counts)[0]))
    got = ctx.kmer_values(c.k)
    assert got.dtype == np.float64
    bad = VC.first_difference(c, got)
    assert bad is None, "%s path: %s" % (VC.path_of(c), bad)
    return got


@pytest.mark.parametrize("name", VC.NAMES)
def test_table_equals_model(ctx, name):
    _run(ctx, VC.case(name))


@pytest.mark.parametrize("names", [
    ("sort-path-k8-palindrome", "tie-at-tile-first-k8", "flat-k6", "sort-path-k8-palindrome"),
    ("edge-of-histogram-k7-T2048", "edge-of-histogram-k7-T2046", "one-tie-falls-k6-T2100", "edge-of-histogram-k7-T2048"),
    ("every-tie-falls-k8-T20", "every-tie-falls-k8-T2100", "edge-of-histogram-k4-T2046", "every-tie-falls-k8-T20"),
], ids=["sort-first-k8", "sort-first-k7", "histogram-first-k8"])
def test_paths_alternate_in_one_context(ctx, names):
    """a table of one path, one of the other path at the same k, one of another k, the first again: nothing of the flag block, the bin
    array or the kept histogram of a call reaches the next"""
    cases = [VC.case(n) for n in names]
    assert cases[0].k == cases[1].k != cases[2].k and VC.path_of(cases[0]) != VC.path_of(cases[1]) and names[3] == names[0]
    first = None
    for c in cases:
        got = _run(ctx, c)
        if first is None:
            first = got
    assert np.array_equal(first.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("name", sorted(VC.CODES, key=VC.CODES.get))
def test_codes(ctx, name):
    """codes[i] = the count of k-mer i where it has a value, 0 where it has none; the flag rises exactly when a VALUED k-mer's count does not
    fit (a cut k-mer's far larger count does not raise it) and the code is clamped there; value_of_code(code, total) gives the table back"""
    import downpore_amd.hip as hip
    c = VC.case(name)
    V = VC.CODES[name]
    _run(ctx, c)
    own = np.where(c.table != 0, c.counts, 0).astype(np.int64)  # what a code stands for
    assert int(own.max()) == V and int(c.counts.max()) >= 3 * V
    for width, last_exact, cap in ((1, 254, 255), (2, 65535, 65535)):
        codes, total, overflow = ctx.values_codes(width)
        assert codes.dtype == (np.uint8 if width == 1 else np.uint16) and codes.shape == c.counts.shape
        assert total == int(c.counts.sum())
        assert overflow == (1 if V > last_exact else 0), (width, V, overflow)
        clamped = own > last_exact
        assert clamped.any() == bool(overflow)
        codes = codes.astype(np.int64)
        assert (codes[clamped] == cap).all(), (width, codes[clamped][:5])
        exact = ~clamped
        assert np.array_equal(codes[exact] == 0, c.table[exact] == 0)
        assert np.array_equal(codes[exact], own[exact])
        lut = M.value_of_code(np.arange(cap + 1), total)  # at most 65 536 evaluations
        rebuilt = lut[codes]
        assert np.array_equal(rebuilt[exact].view(np.uint64), c.table[exact].view(np.uint64))
    # an uploaded table has no histogram behind it
    ctx.values_upload(c.table)
    for width in (1, 2):
        with pytest.raises(hip.DpError):
            ctx.values_codes(width)
