"""The k-mer value table of `downpore overlap` / `downpore map` as a plain numpy model (tests/values_cases.py, tests/test_values_cases_cpu.py on the
CPU, tests/test_gpu_values_table.py on the device).  Test infrastructure only.

Written from the rule, not from dp_values.hip or the host's kmerValuesFromCounts (commands/overlap.go:55-93, util/sequtil/kmers.go:87-112,
DESIGN.md 2 "tie rule"):

* tot = sum of all counts; freq(i) = count(i) / float64(tot); value(i) = 0 for a count below 3, else 1 - (5e-6 - freq) where
  freq <= 5e-6 and 1 - (freq - 5e-6) above it.  float64 throughout, one rounding per operation.
* merged(i) = 2 * count(i) for a k-mer that is its own reverse complement, else 2 * (count(i) + count(rc(i))): what the reference's
  in-place merge loop leaves in both entries of a pair after it has visited each of them.
* topN = 4^k // 100.  T = the merged count at index n - topN of the ascending order.  Every k-mer with merged > T loses its value,
  and of the k-mers with merged == T the topN - #(merged > T) ones with the highest ids.  value(0) = 0.

With the 2-bit code A C G T = 0 1 2 3 and the first base in the top bits, a read of exactly k bases holds exactly one k-mer, so
`reads_of` turns any count table into a read set whose histogram is that table to the letter.
"""
import numpy as np

TARGET_FREQ = 0.000005
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def rc_ids(k):
    """rc(i) of every k-mer id i < 4^k (uint32): complement every 2-bit code and reverse their order"""
    x = ~np.arange(4 ** k, dtype=np.uint32)
    x = ((x >> np.uint32(2)) & np.uint32(0x33333333)) | ((x & np.uint32(0x33333333)) << np.uint32(2))
    x = ((x >> np.uint32(4)) & np.uint32(0x0F0F0F0F)) | ((x & np.uint32(0x0F0F0F0F)) << np.uint32(4))
    x = x.byteswap()
    return x >> np.uint32(32 - 2 * k)


def merged_counts(counts, k):
    """the merged forward + reverse-complement count of every k-mer (int64)"""
    c = np.asarray(counts).astype(np.int64)
    rc = rc_ids(k)
    m = c + c[rc]
    m[rc == np.arange(len(c), dtype=np.uint32)] >>= 1  # (a palindrome is visited once: its own count, not twice it)
    m <<= 1
    return m


def value_of_code(code, total):
    """the value of a k-mer from its own count and the sum of all counts (scalar or array)"""
    code = np.asarray(code)
    out = np.zeros(code.shape, dtype=np.float64)
    valued = code >= 3  # (only these are evaluated: a table at k = 13 is nearly all zeros)
    freq = code[valued].astype(np.float64) / np.float64(total)
    low = np.float64(1.0) - (np.float64(TARGET_FREQ) - freq)
    high = np.float64(1.0) - (freq - np.float64(TARGET_FREQ))
    out[valued] = np.where(freq <= TARGET_FREQ, low, high)
    return out if out.shape else np.float64(out)


def values(counts, k):
    """-> (table float64 [4^k], info): info = dict(n, topN, total, T, above, ties, cut_ties, X); X = the lowest id whose tie is cut.
    T, above, ties, cut_ties and X are None where 4^k // 100 is 0 (no cut)."""
    c = np.asarray(counts).astype(np.int64)
    n = 4 ** k
    assert c.shape == (n,)
    total = int(c.sum())
    table = value_of_code(c, total)
    topN = n // 100
    info = dict(n=n, topN=topN, total=total, T=None, above=None, ties=None, cut_ties=None, X=None)
    if topN > 0:
        merged = merged_counts(c, k)
        # the element at index n - topN of the ascending order; the zeros in front of it need no partitioning
        counted = merged[merged > 0]
        at = n - topN - (n - len(counted))
        T = int(np.partition(counted, at)[at]) if at >= 0 else 0
        above = int(np.count_nonzero(merged > T))
        tie_ids = np.flatnonzero(merged == T)
        ties = len(tie_ids)
        cut_ties = topN - above
        assert 1 <= cut_ties <= ties
        table[merged > T] = 0.0
        table[tie_ids[ties - cut_ties:]] = 0.0
        info.update(T=T, above=above, ties=ties, cut_ties=cut_ties, X=int(tie_ids[ties - cut_ties]))
    table[0] = 0.0
    return table, info


def reads_of(counts, k):
    """-> (ASCII bases, off): counts[i] reads of exactly k bases for every k-mer i, in id order"""
    c = np.asarray(counts).astype(np.int64)
    ids = np.repeat(np.arange(len(c), dtype=np.uint32), c)
    bases = np.empty((len(ids), k), dtype=np.uint8)
    for j in range(k):
        bases[:, j] = _LETTERS[(ids >> np.uint32(2 * (k - 1 - j))) & np.uint32(3)]
    off = np.arange(len(ids) + 1, dtype=np.int64) * k
    return bases.reshape(-1), off
